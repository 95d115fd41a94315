"""rmd_render_ao, rmd_ao_resolve and rmd_ao_buffer_alloc without a GPU: the exports and their arity, every refusal in the header's order with a NULL
context, the rule header under the host sanitizers, the C++ mirror (raymond_cli ao-resolve) against the numpy restatement tests/ao_ref.py bit for bit,
the restatement held to the oracle's render path and told from four wrong readings, the wrappers' C calls on tests/binding_trace.py's recording
stand-in, and the fragility cap of the frames tests/test_gpu_ao.py uses.

The tie to the render path.  On every sample whose first hit is a Diffuse material and whose lobe uniform is < 0.5 — the render then takes the diffuse
lobe —, the object the restatement's AO ray hits is path_obj[1] of orc_trace_sample at bounce_limit 2.  The lobe uniform is the 22-bit uniform of the
block BEFORE the bounce's: block 0 for the pinhole, the accepted lens round's under the thin lens (oracle.cpp: Rng::next3 takes `lobe` from the path's
previous block).  Read as block 0's for every sample, the check cannot hold under a lens: measured on every ninth case, 1,428 of 27,232 such samples
differ, all of them in the lens cases, and none of 27,181 with the previous block's.

The fragility cap.  A sample is fragile if its first hit is (first_hit_ref.fragile_hit), if |t2 - max_distance| <= 1e-9 max_distance, or if the
occluded / open outcome flips under one of fragile_hit's twelve moves of the AO ray.  The GPU test lets at most 3 pixels a frame differ, so a frame
should hold at most 3 pixels with a fragile sample, and 130 of the 158 frames (and the three extra distances) are asserted to.  The two outcome rules
are what max_distance can move: at 1.0 no frame holds more than 1 such pixel, so no case needs 0.5 or 2.0.  The first rule does not depend on
max_distance: 28 frames built around tied or grazing first hits (coincident walls and spheres, two objects sharing one grid, a camera on a wall) hold
10 to 960 pixels with such a sample at any distance — the cap cannot hold for them.  ao_ref.OVER_CAP lists them by exact key with the number measured
for each, which the test asserts as that frame's upper bound, together with 0 pixels by the outcome rules; the feature and ID tests run the same
frames and find the device on the oracle's side of every tie.  No case is dropped, and the GPU test's own rule — at most 3 pixels off, each through one
fragile sample — is the same for every frame.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ao_ref as ref
import first_hit_ref as fr
import oracle_lib as O
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
NEW = {"rmd_ao_buffer_alloc": 4, "rmd_render_ao": 8, "rmd_render_ao_async": 8, "rmd_ao_resolve": 7}  # name -> the header's arity
ALL_KEYS = fr.feature_keys() + fr.feature_keys(lens_edges=True)


def key_ids(keys):
    return [fr.feature_key_id(k) for k in keys]


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
        assert name in open(os.path.join(ROOT, "integration", "gpu.rs")).read()
    assert "#define RMD_ABI_VERSION 6u" in header and abi.RMD_ABI_VERSION == 6  # additions within ABI 6
    assert "#define RMD_AO_WORDS 4u" in header and abi.RMD_AO_WORDS == 4 == ref.WORDS
    assert "occluded + open + none == samples" in header and "modulo 2^32" in header
    fault_list = header.split("RMD_ERR_DEVICE_FAULT = 8", 1)[1].split("*/", 1)[0]  # the calls that wait and report an earlier fault
    assert "rmd_render_ao" in fault_list and "rmd_ao_resolve" in fault_list
    for fn in (render.render_ao, render.ao_resolve, render.render_ao_arrays):
        assert callable(fn)
    assert render.AoBuffer.ALLOC == "rmd_ao_buffer_alloc" and issubclass(render.AoBuffer, render.Framebuffer)
    # no new entry point under a prefix the binding trace must hold a scenario for
    assert not any(n.startswith(("rmd_denoise", "rmd_despike", "rmd_tile_", "rmd_display", "rmd_resolve", "rmd_luminance", "rmd_exposure")) for n in NEW)


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def _rects(*rs):
    arr = (abi.TileRect * max(1, len(rs)))()
    for i, (l, t, w, h) in enumerate(rs):
        arr[i].left, arr[i].top, arr[i].width, arr[i].height = l, t, w, h
    return arr


def test_render_ao_refusals_in_order_without_a_device(product_lib):
    L = product_lib
    cam = scenes.camera(8, 8).pod()
    st = Settings(scenes.camera(8, 8), 4).pod()
    scene = C.c_void_p(0x200000)  # never looked at: every refusal below comes before the context is
    ao = C.c_void_p(0x100000)
    full, outside, overlap = _rects((0, 0, 8, 8)), _rects((4, 4, 4, 5)), _rects((0, 0, 8, 8), (0, 0, 8, 8))
    nan, inf = float("nan"), float("inf")

    def call(fn, sc=scene, c=C.byref(cam), s=C.byref(st), rects=full, n=1, D=1.0, A=ao):
        return fn(None, sc, c, s, rects, n, D, A)

    def refused(word, **kw):
        for fn in (L.rmd_render_ao, L.rmd_render_ao_async):
            assert call(fn, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
            assert word in _last_error(L) and "rmd_render_ao" in _last_error(L), (kw, _last_error(L))

    # 1: scene, camera, settings — each in front of everything after it
    refused("null scene", sc=None, A=None, D=nan, rects=outside)
    refused("null scene", c=None, D=0.0)
    refused("null scene", s=None, rects=None)
    # 2: ao_dev NULL, tiles NULL with n_tiles > 0
    refused("null tiles/ao", A=None, D=nan)
    refused("null tiles/ao", A=None, rects=None, D=-1.0)
    refused("null tiles/ao", rects=None, D=0.0)
    refused("null tiles/ao", A=None, rects=outside)
    # 3: max_distance not > 0, NaN included — in front of the rects
    for bad in (0.0, -0.0, -1.0, -inf, nan):
        refused("max_distance", D=bad)
        refused("max_distance", D=bad, rects=outside)
        refused("max_distance", D=bad, rects=overlap, n=2)
    # 4: first_hit_call's own: a rect outside the frame, two rects that overlap, then the context
    for good in (1.0, 5e-324, inf):
        refused("outside", rects=outside, D=good)
        refused("outside", rects=_rects((0, 0, 8, 8), (0, 0, 8, 9)), n=2, D=good)  # (overlapping too: the frame rule is asked first)
        refused("overlap", rects=overlap, n=2, D=good)
        for kw in ({}, dict(rects=None, n=0), dict(rects=_rects((0, 0, 4, 8), (4, 0, 4, 8)), n=2)):
            for fn in (L.rmd_render_ao, L.rmd_render_ao_async):
                assert call(fn, D=good, **kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
                assert _last_error(L) == "null context", (kw, _last_error(L))
    assert L.rmd_ao_buffer_alloc(None, 8, 8, C.byref(C.c_void_p())) == abi.RMD_ERR_INVALID_ARGUMENT


def test_ao_resolve_refusals_in_order_without_a_device(product_lib):
    L = product_lib
    W, H = 8, 8
    ao, out = C.c_void_p(0x100000), C.c_void_p(0x100000 + W * H * 16)
    inside = C.c_void_p(0x100000 + W * H * 16 - 8)  # the image's first double is the AO buffer's last
    nan, inf = float("nan"), float("inf")

    def call(A=ao, w=W, h=H, v=1.0, M=out, empty=None):
        return L.rmd_ao_resolve(None, A, w, h, v, M, empty)

    def refused(word, **kw):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert word in _last_error(L) and "rmd_ao_resolve" in _last_error(L), (kw, _last_error(L))

    # width or height 0; NULL buffers; empty_value not finite; the ranges overlapping; then the context
    refused("width or height", w=0, A=None, M=None, v=nan)
    refused("width or height", h=0, M=inside, v=inf)
    refused("null ao/out", A=None, v=nan, M=inside)
    refused("null ao/out", M=None, v=inf)
    for bad in (nan, inf, -inf):
        refused("not finite", v=bad)
        refused("not finite", v=bad, M=inside)
    refused("overlaps", M=inside)
    refused("overlaps", M=ao)
    refused("overlaps", M=C.c_void_p(0x100000 - W * H * 8 + 8))  # the image's last double is the AO buffer's first
    empty = C.c_uint64(7)
    for kw in ({}, dict(v=0.0), dict(v=-1e308), dict(empty=C.byref(empty)), dict(M=C.c_void_p(0x100000 - W * H * 8))):
        assert call(**kw) == abi.RMD_ERR_INVALID_ARGUMENT, kw
        assert _last_error(L) == "null context", (kw, _last_error(L))
    assert empty.value == 7  # a refused call writes nothing


# ---------------------------------------------------------------- the rule on hand-made sequences
def test_the_rule_on_hand_made_sequences():
    def run(outcomes, base=None):  # "n" none, "o" open, "x" occluded
        first = np.array([c != "n" for c in outcomes], dtype=bool).reshape(-1, 1, 1)
        occ = np.array([c == "x" for c in outcomes], dtype=bool).reshape(-1, 1, 1)
        return ref.words_from_samples(first, occ, base=None if base is None else np.array(base, dtype=np.uint32).reshape(1, 1, 4)).reshape(4).tolist()

    assert run("") == [0, 0, 0, 0]
    assert run("oxxnoo") == [2, 3, 1, 6]
    assert run("nnn") == [0, 0, 3, 3]
    assert run("xo", base=[0xFFFFFFFF, 0xFFFFFFFF, 5, 3]) == [0, 0, 5, 5]  # modulo 2^32
    for k in range(7):
        assert run("oxxnoo"[k:], base=run("oxxnoo"[:k])) == [2, 3, 1, 6]  # [0, k) then [k, n) == [0, n)
    words = np.array([[2, 3, 1, 6], [0, 0, 3, 3], [0, 0, 0, 0], [5, 0, 0, 5], [0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFE]], dtype=np.uint32)
    out, empty = ref.resolve(words, -2.0)
    assert out.tolist() == [3 / 5, -2.0, -2.0, 0.0, 0.5] and empty == 2


# ---------------------------------------------------------------- the C++ mirror is the restatement
@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def run_cli(cli, tmp_path, words, W, H, *empty_value):
    np.ascontiguousarray(words, dtype="<u4").tofile(str(tmp_path / "ao.u32"))
    r = subprocess.run([cli, "ao-resolve", str(tmp_path / "ao.u32"), str(W), str(H), str(tmp_path / "ao.f64")] + [repr(v) for v in empty_value], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(str(tmp_path / "ao.f64")).reshape(H, W), int(r.stdout.split()[0])


def test_the_cpp_mirror_is_the_restatement_on_random_records(cli, tmp_path):
    W, H = 37, 21
    words = ref.random_records(np.random.default_rng(0xA0), W * H).reshape(H, W, 4)
    flat = words.reshape(-1, 4)
    den = flat[:, 0].astype(np.uint64) + flat[:, 1]
    assert (flat[:, 3] == 0).any() and ((den == 0) & (flat[:, 2] != 0)).any() and (den > 0xFFFFFFFF).any()  # no samples, `none` alone, a sum past 2^32
    assert ((flat[:, 0] == 0) & (flat[:, 1] != 0)).any() and ((flat[:, 1] == 0) & (flat[:, 0] != 0)).any()
    for args in ((), (1.0,), (0.0,), (-3.5,), (1e-300,)):
        want, want_empty = ref.resolve(words, *(args or (1.0,)))
        got, empty = run_cli(cli, tmp_path, words, W, H, *args)
        assert got.tobytes() == want.tobytes() and empty == want_empty == int((den == 0).sum()), args
        assert ((got > 0) & (got < 1)).any() and (got[den.reshape(H, W) != 0] <= 1.0).all()
    zeroed, n = run_cli(cli, tmp_path, np.zeros((H, W, 4), dtype=np.uint32), W, H, 0.25)  # a zeroed buffer
    assert zeroed.tobytes() == np.full((H, W), 0.25).tobytes() and n == W * H
    r = subprocess.run([cli, "ao-resolve", str(tmp_path / "ao.u32"), str(W), str(H), str(tmp_path / "ao.f64"), "nan"], capture_output=True, text=True)
    assert r.returncode == 1 and "not finite" in r.stderr


# ---------------------------------------------------------------- the rule header, on the CPU under the sanitizers
def test_the_rule_header_agrees_with_a_plain_reading_under_sanitizers(tmp_path):
    header = open(os.path.join(CSRC, "ao_rule.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", header) == ["stdint.h"]  # nothing of the project, nothing of HIP
    assert "inline void ao_count(" in header and "inline double ao_resolve_pixel(" in header
    code = re.sub(r"//[^\n]*", "", header.split("namespace rmd {", 1)[1])
    assert not re.search(r"\b(for|while)\b", code) and set(re.findall(r"rec\[(\w+)\]", header)) <= set("0123") | {"kAoWords"}  # every index a constant
    kernel = open(os.path.join(CSRC, "ao.hip")).read()
    shared = open(os.path.join(CSRC, "first_hit.hpp")).read()
    assert '#include "first_hit.hpp"' in kernel and '#include "ao_rule.hpp"' in kernel
    for fn, text in (("ao_count(rec,", kernel), ("ao_resolve_pixel(rec,", kernel), ("scene_intersect_wave<GRID>(", shared), ("if constexpr (sink_second_ray<Sink>::value)", shared)):
        assert fn in text, fn  # the kernels read the same lines
    assert shared.count("scene_intersect_wave<GRID>(") == 2 and "kSecondRay = true" in kernel  # the second segment is the body's, asked for by the sink
    assert "asm" not in kernel and "asm" not in shared and "__shared__" not in kernel  # no new LDS
    for fn in ("onb(", "cosine_hemisphere(", "mat3_mul(", "normalize("):
        assert fn in kernel, fn  # the render kernel's device functions
    mirror = open(os.path.join(ROOT, "raymond_amd", "host", "raymond.cpp")).read()
    assert '#include "../csrc/ao_rule.hpp"' in mirror and "rmd::ao_resolve_pixel(" in mirror  # ... and so does the C++ mirror
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "ao_rule")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "ao_rule_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe, "31", "100000"], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"ao rule ok: (\d+) records, (\d+) near the wrap, (\d+) with a zero denominator, (\d+) strictly between 0 and 1, (\d+) all open, (\d+) all occluded, "
                  r"(\d+) with open \+ occluded past 2\^32", r.stdout)
    assert m and int(m.group(1)) == 100000 and all(int(m.group(i)) > 1000 for i in range(2, 8))


# ---------------------------------------------------------------- the restatement: the oracle's render path, and four wrong readings
TIE_KEYS = ALL_KEYS[::9] + [("spheres", "shuffled_room", 1, True, None), ("mesh", "camera_in_box", 1, True, None), ("spheres", "shuffled_room", 1, False, "aperture-4")]


@pytest.mark.parametrize("key", TIE_KEYS, ids=key_ids(TIE_KEYS))
def test_the_ao_ray_is_the_renders_diffuse_bounce(oracle, product_lib, key):
    fc = fr.feature_case(key)
    S, _ = ref.reference(key)
    osc = O.OracleScene(fc.scene)
    objs = fc.scene.flatten()[0]
    kinds = np.array([objs[i].material.kind for i in range(len(fc.scene.objects))])
    st = Settings(fc.cam, sample_count=fc.spp, bounce_limit=2, seed=fc.seed, use_dof=fc.use_dof)
    spp, H, W = S.first.shape
    checked = 0
    for s in range(spp):
        ys, xs = np.nonzero(S.first[s] & (kinds[np.maximum(S.obj[s], 0)] == abi.RMD_MAT_DIFFUSE))
        pix, smp = ys * W + xs, np.full(len(ys), fc.begin + s, dtype=np.uint32)
        rounds = ref.lens_rounds(fc.cam, fc.seed, fc.use_dof, pix, smp, S.rays[s][ys, xs], ~S.no_ray[s][ys, xs])  # (asserts the lens origins bit for bit)
        lobe = O.block_uniforms(fc.seed, pix, smp, rounds)[:, 2]  # the block before the bounce's: block 0 for the pinhole
        for i in np.flatnonzero(lobe < 0.5)[:400]:
            y, x = int(ys[i]), int(xs[i])
            _, po, _ = osc.trace_sample_path(fc.cam, st, x, y, fc.begin + s)
            assert len(po) >= 2 and int(po[0]) == int(S.obj[s, y, x]) and int(po[1]) == int(S.obj2[s, y, x]), (x, y, s, po.tolist(), int(S.obj2[s, y, x]))
            checked += 1
    print("ao host: %s: %d samples on the render's path" % (fr.feature_key_id(key), checked))
    assert checked > 0 or not (S.first & (kinds[np.maximum(S.obj, 0)] == abi.RMD_MAT_DIFFUSE)).any()


WRONG = {"block0": ("spheres", "shuffled_room", 0, False, None), "normal_first": ("spheres", "shuffled_room", 0, False, None),
         "offset_along_dir": ("spheres", "tilted_pairs", 0, False, None), "skip_no_ray": ("spheres", "shuffled_room", 1, False, "focal-negative")}


def test_the_restatement_is_told_from_four_wrong_readings(oracle):
    assert ref.VARIANTS == ("block0", "offset_along_dir", "normal_first", "skip_no_ray") and set(WRONG) == set(ref.VARIANTS)
    for variant, key in WRONG.items():
        fc = fr.feature_case(key)
        _, right = ref.reference(key, 1.0)
        wrong = ref.frame_words(fc.scene, fc.cam, fc.seed, fc.spp, fc.begin, fc.use_dof, 1.0, variant=variant)
        differ = int((wrong != right).any(axis=2).sum())
        print("ao host: %s changes %d pixels of %s" % (variant, differ, fr.feature_key_id(key)))
        assert differ > 0, variant
        w = wrong.astype(np.uint64)
        assert (w[..., 0] + w[..., 1] + w[..., 2] == w[..., 3]).all()
        if variant == "skip_no_ray":  # no sample of the frame has a ray: counted, every pixel is {none = samples = 6}; skipped, zeros
            assert (right == np.array([0, 0, fc.spp, fc.spp], dtype=np.uint32)).all() and not wrong.any()
        else:
            assert (wrong[..., 3] == fc.spp).all() and (wrong[..., 2] == right[..., 2]).all()  # the first hits are the same: only occluded / open move


AGREE_KEYS = [("spheres", "coincident_spheres", 0, False, None), ("spheres", "camera_on_walls", 0, False, None), ("mesh", "camera_in_box", 2, False, None),
              ("mesh", "shared_grid", 0, False, None), ("spheres", "shuffled_room", 0, False, None)]


@pytest.mark.parametrize("key", AGREE_KEYS, ids=key_ids(AGREE_KEYS))
def test_the_vectorised_first_hit_rule_is_fragile_hit(oracle, product_lib, key):
    """ao_ref.first_hit_fragile (what the cap counts with) against first_hit_ref.fragile_hit (what the GPU accounting asks), sample by sample: every
    sample the vectorised rule calls fragile, and as many it does not, on frames with tied hits, grazing hits and neither"""
    fc = fr.feature_case(key)
    S, _ = ref.reference(key)
    osc = O.OracleScene(fc.scene)
    flat = lambda a: np.ascontiguousarray(a).reshape((-1,) + a.shape[3:])
    rays, obj, t, sub, no_ray = flat(S.rays), flat(S.obj), flat(S.t), flat(S.sub), flat(S.no_ray)
    fast = ref.first_hit_fragile(fc.scene, osc, rays, obj, t, sub, no_ray)
    rng = np.random.default_rng(35)
    yes, no = np.flatnonzero(fast), np.flatnonzero(~fast & ~no_ray)
    picked = np.concatenate([rng.permutation(yes)[:150], rng.permutation(no)[:150]])
    slow = np.array([fr.fragile_hit(fc.scene, osc, rays[i], obj[i], t[i], sub[i]) is not None for i in picked], dtype=bool)
    print("ao host: %s: %d of %d samples fragile by the vectorised rule; %d compared" % (fr.feature_key_id(key), len(yes), len(fast), len(picked)))
    assert (slow == fast[picked]).all(), picked[slow != fast[picked]][:5].tolist()
    assert bool(len(yes)) == (fr.feature_key_id(key) in ref.OVER_CAP)


# ---------------------------------------------------------------- the binding's C calls, on tests/binding_trace.py's recording stand-in
def test_the_signature_table_holds_the_names_render_py_mentions():
    mentioned = set(re.findall(r"\brmd_[a-z0-9_]+\b", open(os.path.join(ROOT, "raymond_amd", "render.py")).read()))
    assert set(NEW) - {"rmd_render_ao_async"} <= mentioned and set(NEW) <= set(lib.SIGNATURES)  # (the _async form is made from its stem: _render_call)


def test_the_wrappers_make_the_calls_with_the_arguments_in_the_headers_order():
    import binding_trace as bt

    with bt.installed() as fake:
        b = bt.Bench()
        try:
            st = Settings(scenes.camera(bt.W, bt.H), 4)
            rects = "[" + ",".join("[%d,%d,%d,%d]" % r for r in bt.RECTS) + "]"
            with render.DeviceScene(b.ctx, scenes.reflective_spheres()) as ds, render.AoBuffer(b.ctx, bt.W, bt.H) as ao:
                assert fake.lines[-1] == "rmd_ao_buffer_alloc(ctx0,8,6,out)" and ao.shape == (bt.H, bt.W, 4)
                ao.ptr, ao.owned = b.fbs[0].ptr, False  # (the stand-in hands out no AO buffers: one of its own stands in)
                render.render_ao(b.ctx, ds, st.camera_settings, st, bt.RECTS, 1.5, ao, 2, 3)
                assert fake.lines[-1].startswith("rmd_render_ao(ctx0,scene0,[") and fake.lines[-1].endswith(",%s,4,1.5,fb0)" % rects)
                render.render_ao(b.ctx, ds, st.camera_settings, st, bt.RECTS, float("inf"), ao, sync=False)
                assert fake.lines[-1].startswith("rmd_render_ao_async(ctx0,scene0,[") and fake.lines[-1].endswith(",%s,4,inf,fb0)" % rects)
                ao.zero()
                assert fake.lines[-1] == "rmd_framebuffer_zero(ctx0,fb0,96)"  # 2 doubles a pixel
                words = ao.download()
                assert fake.lines[-1] == "rmd_framebuffer_download(ctx0,fb0,host,96)" and words.shape == (bt.H, bt.W, 4) and words.dtype == np.uint32
                live = list(fake.live)
                image, empty = render.ao_resolve(b.ctx, ao, 0.25)
                call = next(line for line in reversed(fake.lines) if line.startswith("rmd_ao_resolve("))
                assert re.fullmatch(r"rmd_ao_resolve\(ctx0,fb0,8,6,0\.25,fb\d+,out\)", call)
                assert image.shape == (bt.H, bt.W) and image.dtype == np.float64 and empty == 0 and fake.live == live  # the image's buffer is closed
                render.ao_resolve(b.ctx, ao)
                call = next(line for line in reversed(fake.lines) if line.startswith("rmd_ao_resolve("))
                assert re.fullmatch(r"rmd_ao_resolve\(ctx0,fb0,8,6,1\.0,fb\d+,out\)", call)  # the default: an empty pixel is open
                fake.fail = ("rmd_ao_resolve",)
                with pytest.raises(lib.RaymondError):
                    render.ao_resolve(b.ctx, ao)
                assert fake.live == live
                fake.fail = ()
        finally:
            b.close()
        assert fake.live == []


# ---------------------------------------------------------------- the fragility cap of the GPU test's frames
CAP_CASES = [(k, None) for k in ALL_KEYS] + list(ref.EXTRA_DISTANCES)


@pytest.mark.parametrize("key,distance", CAP_CASES, ids=[fr.feature_key_id(k) + ("" if d is None else "-%r" % d) for k, d in CAP_CASES])
def test_every_frame_holds_at_most_three_pixels_with_a_fragile_sample(oracle, product_lib, key, distance):
    fc = fr.feature_case(key)
    D = ref.case_distance(key) if distance is None else distance
    assert distance is not None or D in (1.0, 0.5, 2.0)
    S, words = ref.reference(key, D)
    every, by_outcome = ref.fragile_pixels(fc.scene, S, D)
    print("ao host: %s at max_distance %g: %d pixels hold a fragile sample, %d by the outcome rules; occluded %d of %d first hits"
          % (fr.feature_key_id(key), D, int(every.sum()), int(by_outcome.sum()), int(S.occluded.sum()), int(S.first.sum())))
    assert int(by_outcome.sum()) <= 3  # what max_distance can move
    # the full cap; a frame of ao_ref.OVER_CAP — fragile first hits by construction, at any distance — is held to the number measured for it instead
    assert int(every.sum()) <= (ref.OVER_CAP.get(fr.feature_key_id(key), 3) if distance is None else 3)
    if distance is None and fr.feature_key_id(key) in ref.OVER_CAP:
        assert int(by_outcome.sum()) == 0 and int(every.sum()) > 3  # (a frame that no longer needs its entry loses it)
    w = words.astype(np.uint64)
    assert (w[..., 0] + w[..., 1] + w[..., 2] == w[..., 3]).all() and (w[..., 3] == fc.spp).all()
