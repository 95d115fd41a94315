"""rmd_render_ids, rmd_ids_matte and rmd_id_buffer_alloc without a GPU: the exports and their arity, every refusal in the header's order with a NULL
context, the rule on hand-made sequences, the C++ mirror (raymond_cli ids-matte: the rule header driven the way the kernel drives it) against the numpy
restatement tests/ids_ref.py bit for bit, the rule header under the host sanitizers, the restatement told from three wrong readings, and the wrappers'
C calls on tests/binding_trace.py's recording stand-in."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ids_ref as ref
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
NEW = {"rmd_id_buffer_alloc": 4, "rmd_render_ids": 7, "rmd_render_ids_async": 7, "rmd_ids_matte": 8}  # name -> the header's arity
MISS = ref.MISS


# ---------------------------------------------------------------- the boundary
def test_the_four_symbols_are_exported_declared_and_in_the_one_table(product_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    header = " ".join(open(os.path.join(ROOT, "include", "raymond_hip.h")).read().split())
    for name, arity in NEW.items():
        assert name in exported and name in lib.SIGNATURES
        decl = re.search(r"rmd_status %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == arity == len(lib.SIGNATURES[name][1]), name
        fn = getattr(product_lib, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == lib.SIGNATURES[name][1]
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "#define RMD_ABI_VERSION 6u" in header and abi.RMD_ABI_VERSION == 6  # additions within ABI 6
    assert "#define RMD_ID_SLOTS 4u" in header and "#define RMD_ID_WORDS 10u" in header and "#define RMD_ID_MISS 0xFFFFFFFFu" in header
    assert (abi.RMD_ID_SLOTS, abi.RMD_ID_WORDS, abi.RMD_ID_MISS) == (4, 10, 0xFFFFFFFF) == (ref.SLOTS, ref.WORDS, ref.MISS)
    assert "modulo 2^32" in header
    for fn in (render.render_ids, render.ids_matte, render.render_ids_arrays, render.ids_ranked):
        assert callable(fn)
    assert render.IdBuffer.ALLOC == "rmd_id_buffer_alloc" and issubclass(render.IdBuffer, render.Framebuffer)
    # no new entry point under a prefix the binding trace must hold a scenario for
    assert not any(n.startswith(("rmd_denoise", "rmd_despike", "rmd_tile_", "rmd_display", "rmd_resolve", "rmd_luminance", "rmd_exposure")) for n in NEW)


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def _rects(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def test_render_ids_refusals_in_order_without_a_device(product_lib):
    L = product_lib
    cam = scenes.camera(8, 8).pod()
    st = Settings(scenes.camera(8, 8), 4).pod()
    scene = C.c_void_p(0x200000)  # never looked at: every refusal below comes before the context is
    ids = C.c_void_p(0x100000)
    full, outside, overlap = _rects((0, 0, 8, 8)), _rects((4, 4, 4, 5)), _rects((0, 0, 8, 8), (0, 0, 8, 8))

    def call(fn, sc=scene, c=C.byref(cam), s=C.byref(st), rects=full, n=1, I=ids):
        return fn(None, sc, c, s, rects, n, I)

    def refused(word, **kw):
        for fn in (L.rmd_render_ids, L.rmd_render_ids_async):
            assert call(fn, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
            assert word in _last_error(L) and "rmd_render_ids" in _last_error(L), (kw, _last_error(L))

    refused("null scene", sc=None)
    refused("null scene", c=None)
    refused("null scene", s=None)
    # the stated order: ids_dev NULL, tiles NULL with n_tiles > 0, a rect outside the frame, two rects that overlap — each in front of those after it
    refused("null tiles/ids", I=None)
    refused("null tiles/ids", I=None, rects=None)
    refused("null tiles/ids", I=None, rects=outside)
    refused("null tiles/ids", rects=None)
    refused("outside", rects=outside)
    refused("outside", rects=_rects((0, 0, 8, 8), (0, 0, 8, 9)), n=2)  # (overlapping too: the frame rule is asked first)
    refused("overlap", rects=overlap, n=2)
    for kw in ({}, dict(rects=None, n=0), dict(rects=_rects((0, 0, 4, 8), (4, 0, 4, 8)), n=2)):
        for fn in (L.rmd_render_ids, L.rmd_render_ids_async):
            assert call(fn, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
            assert _last_error(L) == "null context", (kw, _last_error(L))
    assert L.rmd_id_buffer_alloc(None, 8, 8, C.byref(C.c_void_p())) == abi.RMD_ERR_INVALID_ARGUMENT


def test_ids_matte_refusals_in_order_without_a_device(product_lib):
    L = product_lib
    W, H = 8, 8
    ids, matte = C.c_void_p(0x100000), C.c_void_p(0x100000 + W * H * 40)
    objs = (C.c_uint32 * 4)(0, 3, MISS, 3)
    long_list = (C.c_uint32 * 2049)()
    bad_entry = (C.c_uint32 * 3)(1, 0xFFFFFFFE, 2)
    inside = C.c_void_p(0x100000 + W * H * 40 - 8)  # the matte's first double is the ID buffer's last

    def call(I=ids, w=W, h=H, o=objs, n=4, M=matte, other=None):
        return L.rmd_ids_matte(None, I, w, h, o, n, M, other)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert word in _last_error(L) and "rmd_ids_matte" in _last_error(L), (kw, _last_error(L))

    # width or height 0; NULL buffers; objects NULL with n_objects > 0; a list that is too long; [the entry]; the ranges overlapping; then the context
    refused("width or height", w=0, I=None, o=None, n=9999, M=None)
    refused("width or height", h=0, M=inside)
    refused("null ids/matte", I=None, o=None, n=9999)
    refused("null ids/matte", M=None, o=long_list, n=2049)
    refused("null objects", o=None, n=1, M=inside)
    refused("null objects", o=None, n=4000, M=inside)
    refused("more than 2048", o=long_list, n=2049, M=inside)
    refused("0xFFFFFFFE", o=bad_entry, n=3, M=inside)
    refused("overlaps", M=inside)
    refused("overlaps", M=ids)
    refused("overlaps", M=C.c_void_p(0x100000 - W * H * 8 + 8))  # the matte's last double is the ID buffer's first
    other = C.c_uint64(7)
    for kw in ({}, dict(o=None, n=0), dict(o=long_list, n=2048), dict(other=C.byref(other)), dict(M=C.c_void_p(0x100000 - W * H * 8))):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))
    assert other.value == 7  # a refused call writes nothing


# ---------------------------------------------------------------- the rule on hand-made sequences
def run_rule(keys, base=None):
    """the restatement over one pixel: keys in order (object indices, -1 = a miss) -> its ten words as a list"""
    objs = np.array(keys, dtype=np.int64).reshape(-1, 1, 1)
    return [int(v) for v in ref.words_from_objs(objs, base=None if base is None else np.array(base, dtype=np.uint32).reshape(1, 1, 10)).reshape(10)]


def test_the_rule_on_hand_made_sequences():
    assert run_rule([]) == [0] * 10
    # first-seen order, not key order and not count order; object o has key o + 1, a miss RMD_ID_MISS
    assert run_rule([7, 2, 2, -1, 2, 7]) == [8, 2, 3, 3, MISS, 1, 0, 0, 0, 6]
    # the fifth distinct key goes to `other`, and so does every later new one
    assert run_rule([5, 4, 3, 2, 1]) == [6, 1, 5, 1, 4, 1, 3, 1, 1, 5]
    assert run_rule([5, 4, 3, 2, 1, 0, 1]) == [6, 1, 5, 1, 4, 1, 3, 1, 3, 7]
    # a key seen again after the table is full still finds its slot
    assert run_rule([5, 4, 3, 2, 1, 3, 5, 2]) == [6, 2, 5, 1, 4, 2, 3, 2, 1, 8]
    # the miss takes a slot like an object, and can be the one that overflows
    assert run_rule([-1, -1, 0]) == [MISS, 2, 1, 1, 0, 0, 0, 0, 0, 3]
    assert run_rule([0, 1, 2, 3, -1, -1]) == [1, 1, 2, 1, 3, 1, 4, 1, 2, 6]
    rng = np.random.default_rng(29)
    for _ in range(200):
        n, pool = int(rng.integers(0, 30)), int(rng.integers(1, 9))
        keys = [int(k) for k in rng.integers(-1, pool, n)]
        w = run_rule(keys)
        assert sum(w[1:8:2]) + w[8] == w[9] == n  # sum + other == samples
        used = [k for k in w[0:8:2] if k]
        assert w[0:8:2] == used + [0] * (4 - len(used))  # empty slots trail
        firsts = list(dict.fromkeys(int(ref.key_of(k)) for k in keys))
        assert used == firsts[:4] and (w[8] != 0) == (len(firsts) > 4)  # first-seen order
        k = int(rng.integers(0, n + 1))
        assert run_rule(keys[k:], base=run_rule(keys[:k])) == w  # [0, k) then [k, n) == [0, n)
    # counts are modulo 2^32
    assert run_rule([3], base=[4, 0xFFFFFFFF, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF]) == [4, 0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0]


def test_ids_ranked_orders_by_count_then_slot():
    words = np.array([[[8, 2, 3, 3, MISS, 1, 0, 0, 0, 6], [6, 1, 5, 4, 4, 1, 3, 4, 1, 11]]], dtype=np.uint32)
    keys, counts = render.ids_ranked(words)
    assert keys.shape == counts.shape == (1, 2, 4)
    assert keys[0, 0].tolist() == [3, 8, MISS, 0] and counts[0, 0].tolist() == [3, 2, 1, 0]
    assert keys[0, 1].tolist() == [5, 3, 6, 4] and counts[0, 1].tolist() == [4, 4, 1, 1]  # ties by slot


# ---------------------------------------------------------------- the C++ mirror is the restatement
@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def run_cli(cli, tmp_path, words, W, H, listing):
    np.ascontiguousarray(words, dtype="<u4").tofile(str(tmp_path / "ids.u32"))
    r = subprocess.run([cli, "ids-matte", str(tmp_path / "ids.u32"), str(W), str(H), listing, str(tmp_path / "matte.f64")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(str(tmp_path / "matte.f64")).reshape(H, W), int(r.stdout.split()[0])


LISTS = (("7", [7]), ("3,miss,3,7,12,3", [3, MISS, 3, 7, 12, 3]), ("miss", [MISS]), ("none", []), ("1000,2000", [1000, 2000]),
         (",".join(str(i) for i in range(39)) + ",miss", list(range(39)) + [MISS]))


def test_the_cpp_mirror_is_the_restatement_on_random_records(cli, tmp_path):
    W, H = 37, 21
    words = ref.random_records(np.random.default_rng(0x1D5), W * H).reshape(H, W, 10)
    flat = words.reshape(-1, 10)
    assert (flat[:, 9] == 0).any() and ((flat[:, 6] != 0) & (flat[:, 8] == 0)).any() and (flat[:, 8] != 0).any()  # samples == 0, full tables, other
    assert (flat[:, 0:8:2] == MISS).any() and (flat[:, 1:8:2] > 0x7FFFFFFF).any()  # the miss key, counts past 2^31
    seen_between = False
    for listing, objects in LISTS:
        want, want_other = ref.matte(words, objects)
        got, other = run_cli(cli, tmp_path, words, W, H, listing)
        assert got.tobytes() == want.tobytes() and other == want_other == int((flat[:, 8] != 0).sum()), listing
        seen_between |= bool(((got > 0) & (got < 1)).any())
        if not objects or objects == [1000, 2000]:
            assert not got.any()  # the empty list, and a list naming no object of the frame: zeros
    assert seen_between
    zeroed, zeroed_other = run_cli(cli, tmp_path, np.zeros((H, W, 10), dtype=np.uint32), W, H, "0,miss")  # a zeroed buffer
    assert zeroed.tobytes() == np.zeros((H, W)).tobytes() and zeroed_other == 0
    run_cli(cli, tmp_path, words, W, H, "none")  # (ids.u32 holds the random records again)
    full_set, _ = run_cli(cli, tmp_path, words, W, H, LISTS[-1][0])
    reachable = (flat[:, 8] == 0) & (flat[:, 9] != 0) & (flat[:, 1:8:2].astype(np.uint64).sum(axis=1) == flat[:, 9])
    assert reachable.any() and (full_set.reshape(-1)[reachable] == 1.0).all()  # every key in the set, no overflow: exactly 1
    r = subprocess.run([cli, "ids-matte", str(tmp_path / "ids.u32"), str(W), str(H), "4294967294", str(tmp_path / "matte.f64")], capture_output=True, text=True)
    assert r.returncode == 1 and "0xFFFFFFFE" in r.stderr


# ---------------------------------------------------------------- the rule header, on the CPU under the sanitizers
def test_the_rule_header_agrees_with_a_plain_reading_under_sanitizers(tmp_path):
    header = open(os.path.join(CSRC, "ids_rule.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", header) == ["stdint.h"]  # nothing of the project, nothing of HIP
    body = header.split("inline void ids_insert", 1)[1].split("// Whether", 1)[0]
    assert not re.search(r"\b(for|while)\b", body) and set(re.findall(r"rec\[(\w+)\]", body)) <= set("01234567") | {"kIdWords", "kIdOther", "kIdSamples"}  # unrolled: every index a constant
    kernel = open(os.path.join(CSRC, "ids.hip")).read()
    shared = open(os.path.join(CSRC, "first_hit.hpp")).read()  # the first-hit passes' shared body: ids.hip is its ID sink, and the matte kernel
    assert '#include "first_hit.hpp"' in kernel
    for fn, text in (("ids_insert(rec,", kernel), ("ids_matte_pixel(rec,", kernel), ("scene_intersect_wave<GRID>(", shared)):
        assert fn in text, fn  # the kernels read the same lines
    assert "asm" not in kernel and "asm" not in shared
    mirror = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp")).read()
    assert '#include "../csrc/ids_rule.hpp"' in mirror and "rmd::ids_matte_pixel(" in mirror  # ... and so does the C++ mirror
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "ids_rule")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "ids_rule_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe, "29", "100000"], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"ids rule ok: (\d+) sequences, (\d+) with other, (\d+) with a full table, (\d+) without samples, (\d+) set entries naming the miss, "
                  r"(\d+) mattes strictly between 0 and 1, (\d+) near the wrap", r.stdout)
    assert m and int(m.group(1)) == 100000 and all(int(m.group(i)) > 1000 for i in range(2, 8))


# ---------------------------------------------------------------- the restatement against three wrong readings of the definition
def test_the_restatement_is_told_from_three_wrong_readings():
    assert ref.VARIANTS == ("sorted_by_key", "other_in_matte", "skip_no_ray")
    # two pixels: one sees objects 7, 2, 2 and a no-ray sample; the other six distinct things
    objs = np.array([[7, 5], [2, 4], [2, 3], [-1, 2], [7, 1], [2, -1]], dtype=np.int64).reshape(6, 1, 2)
    no_ray = np.zeros((6, 1, 2), dtype=bool)
    no_ray[3, 0, 0] = True
    right = ref.words_from_objs(objs, no_ray=no_ray)
    assert right[0, 0].tolist() == [8, 2, 3, 3, MISS, 1, 0, 0, 0, 6] and right[0, 1].tolist() == [6, 1, 5, 1, 4, 1, 3, 1, 2, 6]
    by_key = ref.words_from_objs(objs, no_ray=no_ray, variant="sorted_by_key")
    assert by_key[0, 0].tolist() == [3, 3, 8, 2, MISS, 1, 0, 0, 0, 6] and by_key.tobytes() != right.tobytes()
    skipped = ref.words_from_objs(objs, no_ray=no_ray, variant="skip_no_ray")
    assert skipped[0, 0].tolist() == [8, 2, 3, 3, 0, 0, 0, 0, 0, 5] and skipped[0, 1].tolist() == right[0, 1].tolist()
    m, other = ref.matte(right, [5, 4])
    assert m[0].tolist() == [0.0, 2 / 6] and other == 1
    wrong, _ = ref.matte(right, [5, 4], variant="other_in_matte")
    assert wrong[0].tolist() == [0.0, 4 / 6]
    # alpha with the no-ray sample counted as a miss: 5 of 6 samples show an object
    assert (1.0 - ref.matte(right, [MISS])[0])[0, 0] == 1.0 - 1 / 6 and (1.0 - ref.matte(skipped, [MISS])[0])[0, 0] == 1.0
    # ... and on random sequences
    rng = np.random.default_rng(34)
    objs = rng.integers(-1, 7, (12, 9, 11))
    no_ray = (objs == -1) & (rng.random(objs.shape) < 0.5)
    right = ref.words_from_objs(objs, no_ray=no_ray)
    for variant in ("sorted_by_key", "skip_no_ray"):
        assert ref.words_from_objs(objs, no_ray=no_ray, variant=variant).tobytes() != right.tobytes(), variant
    assert (right[..., 8] != 0).any() and ref.matte(right, [0, 1], variant="other_in_matte")[0].tobytes() != ref.matte(right, [0, 1])[0].tobytes()


# ---------------------------------------------------------------- the binding's C calls, on tests/binding_trace.py's recording stand-in
def test_the_signature_table_is_the_only_one_and_holds_the_names_render_py_mentions():
    mentioned = set(re.findall(r"\brmd_[a-z0-9_]+\b", open(os.path.join(ROOT, "raymond_amd", "render.py")).read()))
    assert set(NEW) - {"rmd_render_ids_async"} <= mentioned and set(NEW) <= set(lib.SIGNATURES)  # (the _async form is made from its stem: _render_call)
    tables = [n for n, v in vars(lib).items() if isinstance(v, dict) and any(isinstance(k, str) and k.startswith("rmd_") for k in v)]
    assert tables == ["SIGNATURES"]


def test_the_wrappers_make_the_calls_with_the_arguments_in_the_headers_order():
    import binding_trace as bt

    with bt.installed() as fake:
        b = bt.Bench()
        try:
            st = Settings(scenes.camera(bt.W, bt.H), 4)
            rects = "[" + ",".join("[%d,%d,%d,%d]" % r for r in bt.RECTS) + "]"
            with render.DeviceScene(b.ctx, scenes.reflective_spheres()) as ds, render.IdBuffer(b.ctx, bt.W, bt.H) as ids:
                assert fake.lines[-1] == "rmd_id_buffer_alloc(ctx0,8,6,out)" and ids.shape == (bt.H, bt.W, 10)
                ids.ptr, ids.owned = b.fbs[0].ptr, False  # (the stand-in hands out no ID buffers: one of its own stands in)
                render.render_ids(b.ctx, ds, st.camera_settings, st, bt.RECTS, ids, 2, 3)
                assert fake.lines[-1].startswith("rmd_render_ids(ctx0,scene0,[") and fake.lines[-1].endswith(",%s,4,fb0)" % rects)
                render.render_ids(b.ctx, ds, st.camera_settings, st, bt.RECTS, ids, sync=False)
                assert fake.lines[-1].startswith("rmd_render_ids_async(ctx0,scene0,[") and fake.lines[-1].endswith(",%s,4,fb0)" % rects)
                ids.zero()
                assert fake.lines[-1] == "rmd_framebuffer_zero(ctx0,fb0,240)"  # 5 doubles a pixel
                words = ids.download()
                assert fake.lines[-1] == "rmd_framebuffer_download(ctx0,fb0,host,240)" and words.shape == (bt.H, bt.W, 10) and words.dtype == np.uint32
                live = list(fake.live)
                matte, other = render.ids_matte(b.ctx, ids, [3, MISS, 3])
                call = next(line for line in reversed(fake.lines) if line.startswith("rmd_ids_matte("))
                assert re.fullmatch(r"rmd_ids_matte\(ctx0,fb0,8,6,\[3,4294967295,3\],3,fb\d+,out\)", call)
                assert matte.shape == (bt.H, bt.W) and matte.dtype == np.float64 and other == 0 and fake.live == live  # the matte's buffer is closed
                render.ids_matte(b.ctx, ids, [])
                call = next(line for line in reversed(fake.lines) if line.startswith("rmd_ids_matte("))
                assert re.fullmatch(r"rmd_ids_matte\(ctx0,fb0,8,6,0,0,fb\d+,out\)", call)  # the empty list: NULL, 0
                fake.fail = ("rmd_ids_matte",)
                with pytest.raises(lib.RaymondError):
                    render.ids_matte(b.ctx, ids, [1])
                assert fake.live == live
                fake.fail = ()
        finally:
            b.close()
        assert fake.live == []
