"""rmd_intersect_rays, its forms, rmd_camera_rays and the two buffer allocators without a GPU: the exports and the record's layout from a compiled C
program, every refusal of every entry point in the header's order with a NULL context, the Python wrappers' C calls on tests/binding_trace.py's recording
stand-in, the launch plan header under the host sanitizers (a program of its own: tests/rays_plan_main.cpp), the expected records and ray sets of
tests/rays_ref.py — each set checked to be what it names, and the composition told from three wrong readings —, and raymond_cli's argument handling."""
import contextlib
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import first_hit_ref as fr
import rays_ref as ref
from raymond_amd import abi, lib, render, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymond_amd", "csrc")
CLI = os.path.join(ROOT, "raymond_amd", "host", "raymond_cli")
NEW = {"rmd_ray_buffer_alloc": 3, "rmd_hit_buffer_alloc": 3, "rmd_intersect_rays": 5, "rmd_intersect_rays_async": 5, "rmd_intersect_rays_host": 5,
       "rmd_camera_rays": 6}  # name -> the header's arity
MIN_TRIANGLE_HITS = 30000  # rays of the sets that must hit a triangle (measured: 26,512 in (b) and 8,159 in (a), before (c) adds its own)


# ---------------------------------------------------------------- 1: the boundary
def test_the_symbols_are_exported_declared_and_in_the_one_table(product_lib):
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
    assert "#define RMD_RAY_DOUBLES 6u" in header and abi.RMD_RAY_DOUBLES == 6
    assert "#define RMD_HIT_DOUBLES 5u" in header and abi.RMD_HIT_DOUBLES == 5
    assert "#define RMD_MAX_RAYS (1ull << 30)" in header and abi.RMD_MAX_RAYS == 1 << 30
    assert "rmd_ray_buffer_free" not in header and "rmd_hit_buffer_free" not in header and "rmd_framebuffer_free, which frees any device block" in header
    probe_names = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "rmd_probe" not in probe_names  # the product exports no probe
    for fn in (render.intersect_rays, render.intersect_rays_dev, render.intersect_rays_dev_async, render.camera_rays, render.pick):
        assert callable(fn)
    mentioned = set(re.findall(r"\brmd_[a-z0-9_]+\b", open(os.path.join(ROOT, "raymond_amd", "render.py")).read()))
    assert set(NEW) <= mentioned
    assert not any(n.startswith(("rmd_denoise", "rmd_despike", "rmd_tile_", "rmd_display", "rmd_resolve", "rmd_luminance", "rmd_exposure")) for n in NEW)


def test_the_record_layout_matches_the_c_header(tmp_path):
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "raymond_hip.h"
#define O(f) printf(#f " %zu\n", offsetof(rmd_ray_hit, f))
int main(void) {
  printf("sizeof %zu\n", sizeof(rmd_ray_hit));
  printf("ray_doubles %u\nhit_doubles %u\nmax_rays %llu\n", RMD_RAY_DOUBLES, RMD_HIT_DOUBLES, (unsigned long long)RMD_MAX_RAYS);
  O(t); O(normal); O(object); O(triangle);
  return 0; }
"""
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    layout = dict((l.split()[0], int(l.split()[1])) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if l.strip())
    assert layout.pop("sizeof") == C.sizeof(abi.RayHit) == 40 == render.HIT_DTYPE.itemsize == 8 * abi.RMD_HIT_DOUBLES
    assert layout.pop("ray_doubles") == abi.RMD_RAY_DOUBLES and layout.pop("hit_doubles") == abi.RMD_HIT_DOUBLES and layout.pop("max_rays") == abi.RMD_MAX_RAYS
    assert layout == {"t": 0, "normal": 8, "object": 32, "triangle": 36}
    assert [name for name, _ in abi.RayHit._fields_] == list(layout) == list(render.HIT_DTYPE.names)
    for name, offset in layout.items():
        assert getattr(abi.RayHit, name).offset == offset == render.HIT_DTYPE.fields[name][1], name
    assert render.HIT_DTYPE["object"] == np.dtype("<i4") and render.HIT_DTYPE["triangle"] == np.dtype("<u4") and render.HIT_DTYPE["normal"].shape == (3,)
    miss = ref.MISS.tobytes()
    assert miss == np.zeros(4).tobytes() + np.array([-1], dtype="<i4").tobytes() + np.array([0], dtype="<u4").tobytes()  # the 40 stated bytes


def _last_error(L):
    return (L.rmd_last_error(None) or b"").decode()


def test_refusals_in_order_without_a_device(product_lib):
    L = product_lib
    scene, rays, hits = C.c_void_p(0x200000), C.c_void_p(0x100000), C.c_void_p(0x300000)  # never looked at: every refusal below comes before the context is
    too_many = abi.RMD_MAX_RAYS + 1
    for name in ("rmd_intersect_rays", "rmd_intersect_rays_async", "rmd_intersect_rays_host"):
        fn = getattr(L, name)

        def refused(word, sc=scene, r=rays, n=64, h=hits):
            assert fn(None, sc, r, n, h) == abi.RMD_ERR_INVALID_ARGUMENT, (name, word)
            said = name.replace("_async", "") + ": " if word != "null context" else ""  # (the _async form speaks under its stem, as the sibling calls do)
            assert _last_error(L) == said + word or (word == "RMD_MAX_RAYS" and _last_error(L) == said + "more than RMD_MAX_RAYS rays"), (name, word, _last_error(L))

        # 1: NULL pointers — in front of the count and of the context; a NULL buffer is a refusal only with rays to serve
        refused("null pointer", sc=None, n=too_many)
        refused("null pointer", sc=None, r=None, h=None, n=0)
        refused("null pointer", r=None, n=too_many)
        refused("null pointer", h=None)
        refused("null pointer", r=None, h=None, n=1)
        # 2: more than RMD_MAX_RAYS
        refused("RMD_MAX_RAYS", n=too_many)
        refused("RMD_MAX_RAYS", n=2**64 - 1)
        # then the context (the scene's own refusals need one)
        for kw in (dict(), dict(n=abi.RMD_MAX_RAYS), dict(n=1), dict(r=None, h=None, n=0), dict(r=None, n=0)):
            refused("null context", **kw)

    cam = scenes.camera(8, 6).pod()
    xy = np.array([[0, 0], [7, 5], [3, 2]], dtype=np.uint32)
    uv = np.full((3, 2), 0.5)

    def camera_refused(word, c=cam, p=xy, u=uv, n=3, r=rays):
        status = L.rmd_camera_rays(None, None if c is None else C.byref(c), None if p is None else p.ctypes.data_as(C.c_void_p),
                                   None if u is None else u.ctypes.data_as(C.c_void_p), n, r)
        assert status == abi.RMD_ERR_INVALID_ARGUMENT, word
        assert word in _last_error(L) and ("rmd_camera_rays" if word != "null context" else "") in _last_error(L), (word, _last_error(L))

    zero_w, zero_h, wide = scenes.camera(8, 6).pod(), scenes.camera(8, 6).pod(), scenes.camera(8, 6).pod()
    zero_w.backbuffer_width, zero_h.backbuffer_height, wide.backbuffer_width = 0, 0, 65536
    outside_x, outside_y = np.array([[0, 0], [8, 5], [3, 2]], dtype=np.uint32), np.array([[0, 0], [7, 5], [3, 6]], dtype=np.uint32)
    camera_refused("null pointer", c=None, n=too_many)
    camera_refused("null pointer", p=None, c=zero_w)
    camera_refused("null pointer", r=None, p=outside_x)
    camera_refused("RMD_MAX_RAYS", n=too_many, c=zero_w)  # (the pixels are not read)
    camera_refused("backbuffer size", c=zero_w, p=outside_x)
    camera_refused("backbuffer size", c=zero_h)
    camera_refused("backbuffer size", c=wide)
    camera_refused("backbuffer size", c=zero_w, p=None, r=None, n=0)
    camera_refused("pixel outside", p=outside_x)
    camera_refused("pixel outside", p=outside_y, u=None)
    for kw in (dict(), dict(u=None), dict(p=None, r=None, n=0), dict(p=outside_x, n=1)):
        camera_refused("null context", **kw)

    out = C.c_void_p(0x1234)
    for fn in (L.rmd_ray_buffer_alloc, L.rmd_hit_buffer_alloc):
        for n, o in ((0, C.byref(out)), (too_many, C.byref(out)), (64, None)):
            assert fn(None, n, o) == abi.RMD_ERR_INVALID_ARGUMENT and "bad argument" in _last_error(L)
        assert fn(None, 64, C.byref(out)) == abi.RMD_ERR_INVALID_ARGUMENT and _last_error(L) == "null context"
    assert out.value == 0x1234  # a refused call writes nothing


# ---------------------------------------------------------------- the binding's C calls, on tests/binding_trace.py's recording stand-in
@contextlib.contextmanager
def stand_in():
    """binding_trace.installed() with the two allocators handing out labels (`rays0`, `hits0`) — the stand-in's own table names neither"""
    import binding_trace as bt

    added = {"rmd_ray_buffer_alloc": "rays", "rmd_hit_buffer_alloc": "hits"}
    assert not set(added) & set(bt._HANDLES)
    bt._HANDLES.update(added)
    try:
        with bt.installed() as fake:
            yield bt, fake
    finally:
        for name in added:
            del bt._HANDLES[name]


def test_the_wrappers_make_the_calls_with_the_arguments_in_the_headers_order():
    with stand_in() as (bt, fake):
        ctx = render.Context(0)
        try:
            cam = scenes.camera(bt.W, bt.H)
            with render.DeviceScene(ctx, scenes.reflective_spheres()) as ds, render.RayBuffer(ctx, 70) as rays, render.HitBuffer(ctx, 70) as hits:
                assert fake.lines[-2:] == ["rmd_ray_buffer_alloc(ctx0,70,out)", "rmd_hit_buffer_alloc(ctx0,70,out)"]
                assert (rays.n, hits.n) == (420, 350)
                render.intersect_rays_dev(ctx, ds, rays, hits)
                assert fake.lines[-1] == "rmd_intersect_rays(ctx0,scene0,rays0,70,hits0)"
                render.intersect_rays_dev(ctx, ds, rays, hits, n=65)
                assert fake.lines[-1] == "rmd_intersect_rays(ctx0,scene0,rays0,65,hits0)"
                render.intersect_rays_dev_async(ctx, ds, rays, hits)
                assert fake.lines[-1] == "rmd_intersect_rays_async(ctx0,scene0,rays0,70,hits0)"
                render.intersect_rays_dev(ctx, ds, rays, hits, n=1, sync=False)
                assert fake.lines[-1] == "rmd_intersect_rays_async(ctx0,scene0,rays0,1,hits0)"
                rays.upload(np.zeros((70, 6)))
                assert fake.lines[-1] == "rmd_framebuffer_upload(ctx0,host,rays0,420)"
                got = hits.download()
                assert fake.lines[-1] == "rmd_framebuffer_download(ctx0,hits0,host,350)" and got.dtype == render.HIT_DTYPE and got.shape == (70,)
                assert rays.download().shape == (70, 6)
                live = list(fake.live)
                h = render.intersect_rays(ctx, ds, np.zeros((3, 6)))
                assert fake.lines[-1] == "rmd_intersect_rays_host(ctx0,scene0,host,3,host)" and fake.live == live
                assert isinstance(h, render.Hits) and h._fields == ("object", "triangle", "t", "normal")
                assert (h.object.dtype, h.triangle.dtype, h.t.dtype, h.normal.shape) == (np.int32, np.uint32, np.float64, (3, 3))
                assert h.object.base is h.t.base is h.normal.base is h.triangle.base  # views of one structured download
                n_lines = len(fake.lines)
                assert len(render.intersect_rays(ctx, ds, np.zeros((0, 6))).object) == 0 and len(fake.lines) == n_lines  # no rays: no call
                with render.camera_rays(ctx, cam, [[1, 2], [7, 5]]) as made:
                    assert fake.lines[-2] == "rmd_ray_buffer_alloc(ctx0,2,out)"
                    assert re.fullmatch(r"rmd_camera_rays\(ctx0,\[8,6,.*\],host,0,2,rays1\)", fake.lines[-1]), fake.lines[-1]
                    render.camera_rays(ctx, cam, [[1, 2]], uv=[[0.25, 0.75]], out=made)
                    assert re.fullmatch(r"rmd_camera_rays\(ctx0,\[8,6,.*\],host,host,1,rays1\)", fake.lines[-1]), fake.lines[-1]
                assert fake.live == live
                at = len(fake.lines)
                obj, tri, t, normal = render.pick(ctx, ds, cam, 3, 4)
                calls = [line.split("(", 1)[0] for line in fake.lines[at:]]
                assert calls == ["rmd_ray_buffer_alloc", "rmd_camera_rays", "rmd_hit_buffer_alloc", "rmd_intersect_rays", "rmd_framebuffer_download", "rmd_framebuffer_free",
                                 "rmd_framebuffer_free"], calls
                assert re.fullmatch(r"rmd_intersect_rays\(ctx0,scene0,rays\d+,1,hits\d+\)", fake.lines[at + 3])  # the ray never leaves the device
                assert isinstance(obj, int) and isinstance(tri, int) and isinstance(t, float) and normal.shape == (3,) and fake.live == live
                fake.fail = ("rmd_camera_rays",)
                with pytest.raises(lib.RaymondError):
                    render.camera_rays(ctx, cam, [[1, 2]])
                with pytest.raises(lib.RaymondError):
                    render.pick(ctx, ds, cam, 0, 0)
                fake.fail = ("rmd_intersect_rays",)
                with pytest.raises(lib.RaymondError):
                    render.pick(ctx, ds, cam, 0, 0)
                assert fake.live == live  # a failing call leaves no buffer behind
                fake.fail = ()
        finally:
            ctx.close()
        assert fake.live == []


# ---------------------------------------------------------------- 2: the launch plan header, on the CPU under the sanitizers
def test_the_launch_plan_partitions_the_batches_under_sanitizers(tmp_path):
    header = open(os.path.join(CSRC, "rays_plan.hpp")).read()
    assert re.findall(r"#include [<\"]([^>\"]+)[>\"]", header) == ["stdint.h"]  # nothing of the project, nothing of HIP
    kernel, host = open(os.path.join(CSRC, "rays.hip")).read(), open(os.path.join(CSRC, "api_rays.cpp")).read()
    assert '#include "rays_plan.hpp"' in kernel and "rays_plan(n_rays, n_cus, L.waves_per_wg)" in kernel  # the launcher reads it
    assert "for (uint32_t b = unit; b < n_batches; b += total_waves)" in kernel  # the loop the program walks
    assert "scene_intersect_wave<GRID>(" in kernel and "/*arbitrary_rays=*/true, P.visit_mask)" in kernel and "stage_scene_tables<GRID>(" in kernel
    assert "asm" not in kernel and '#include "rays_plan.hpp"' in host
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "rays_plan")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "rays_plan_main.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"rays plan ok: (\d+) plans, (\d+) batches walked, (\d+) with waves that loop, largest n (\d+)", r.stdout)
    assert m and int(m.group(1)) > 12 * 1026 and int(m.group(3)) > 100 and int(m.group(4)) == 1 << 30


# ---------------------------------------------------------------- 3: the expected records and the ray sets
def _all_sets():
    return [("a", n) for n in ref.ROOMS] + [("b", k) for k in ref.keys_b()] + [("c", k) for k in ref.keys_c()] + [("d", n) for n in ref.TABLES]


def test_the_ray_sets_are_what_they_name(oracle, product_lib):
    keys_b, keys_c = ref.keys_b(), ref.keys_c()
    # (b): every case of the two scene modules at the small frames, the lens variants among them, each a batch of at least 960 rays
    import mesh_scenes as ms
    import sphere_scenes as ss

    small = lambda mod, kind: [(kind,) + tuple(c) + (None,) for c in mod.cases() if (mod.build(c)[1].backbuffer_width, mod.build(c)[1].backbuffer_height) in ref.SMALL_FRAMES]
    assert keys_b == small(ss, "spheres") + small(ms, "mesh") and len(keys_b) == 119 and sum(k[3] for k in keys_b) > 10
    # (c): the grid at object 63, 64 and 70 and on both sides of 64; three grids; NaN normals
    positions = {k[2]: ms.grid_objects(fr.feature_case(k).scene) for k in keys_c if k[1] == "grid_positions"}
    assert positions == {2: [63], 3: [64], 4: [70], 5: [62, 66]}
    assert sum(k[1] == "three_grids" for k in keys_c) == 4 and sum(k[1] == "nan_normals" for k in keys_c) == 2 and len(keys_c) == 10
    assert all(len(ms.grid_objects(fr.feature_case(k).scene)) >= 3 for k in keys_c if k[1] == "three_grids")
    kinds_hit, misses, on_triangles, nan_normals, n_rays = set(), 0, 0, 0, 0
    for kind, key in _all_sets():
        rs, recs = ref.reference(kind, key)
        kinds = ref._kinds(rs.scene)
        assert len(rs.batches) == len(recs)
        if kind == "a":  # the probe test's own batches: ten classes and the shuffled one, whole waves
            assert [b[0] for b in rs.batches] == list(ref.grid_rays.CLASSES) + ["shuffled"] and all(len(b[1]) % 64 == 0 for b in rs.batches)
            assert kinds[1] == 2 and (kinds == 0).sum() == 6  # the grid in its room
        if kind == "b":
            cam = fr.feature_case(key).cam
            n_pixels = cam.backbuffer_width * cam.backbuffer_height
            primary_hits = int((recs[0]["object"][:n_pixels] >= 0).sum())
            assert n_pixels >= 960 and len(rs.batches[0][1]) == n_pixels + primary_hits
            o = rs.batches[0][1][n_pixels:]
            norm = np.sqrt((o[:, 3:] ** 2).sum(axis=1))
            assert np.abs(norm - 1.0).max(initial=0.0) < 1e-15 and (primary_hits == 0 or (o[:, 3:].min(axis=0) < 0).all() and (o[:, 3:].max(axis=0) > 0).all())  # the whole sphere
        if kind == "c":
            assert len(rs.batches) == 1 + len(ms.distinct_grids(rs.scene)) and all(len(b[1]) == ref.K_GRID * len(ref.grid_rays.CLASSES) for b in rs.batches[1:])
        if kind == "d":
            assert len(rs.scene.objects) == key and len(np.unique(recs[0]["object"])) > 100  # the table's spheres are seen
        for (label, rays), rec in zip(rs.batches, recs):
            assert rays.shape == (len(rec), 6) and not rays.flags.writeable and not rec.flags.writeable
            hit = rec["object"] >= 0
            assert rec[~hit].tobytes() == ref.MISS.tobytes() * int((~hit).sum())  # a miss is the 40 stated bytes
            assert not rec["triangle"][hit & (kinds[np.maximum(rec["object"], 0)] != 2)].any()
            kinds_hit |= set(kinds[rec["object"][hit]].tolist())
            misses += int((~hit).sum())
            on_triangles += int((hit & (kinds[np.maximum(rec["object"], 0)] == 2)).sum())
            nan_normals += int(np.isnan(rec["normal"]).any(axis=1).sum())
            n_rays += len(rec)
            if rs.label.startswith("b/open_scene"):
                assert (~hit).sum() > 100  # misses occur
    print("rays host: %d rays in %d sets: %d misses, %d on a triangle, %d with a NaN normal" % (n_rays, len(_all_sets()), misses, on_triangles, nan_normals))
    assert kinds_hit == {0, 1, 2} and misses > 1000 and on_triangles > MIN_TRIANGLE_HITS and nan_normals > 0


WRONG = {"higher_index_wins_ties": ("b", ("spheres", "coincident_spheres", 0, False, None)), "normal_at_origin": ("b", ("spheres", "shuffled_room", 1, False, None)),
         "triangle_kept_off_the_mesh": ("a", "monkeysmooth")}


def test_the_composition_is_told_from_three_wrong_readings(oracle, product_lib):
    assert set(WRONG) == set(ref.VARIANTS)
    for variant, (kind, key) in WRONG.items():
        rs, recs = ref.reference(kind, key)
        kinds = ref._kinds(rs.scene)
        differ = on_planes = 0
        for (_, rays), right in zip(rs.batches, recs):
            wrong = ref.expected_records(rs.scene, rays, variant=variant)
            off = np.array([wrong[i].tobytes() != right[i].tobytes() for i in range(len(right))])
            differ += int(off.sum())
            if variant == "higher_index_wins_ties":  # the same distance, a higher index
                assert (wrong["object"][off] > right["object"][off]).all() and np.array_equal(wrong["t"][off], right["t"][off])
            elif variant == "normal_at_origin":  # only normals move, and only on spheres: a plane's is stored
                assert np.array_equal(wrong["object"], right["object"]) and np.array_equal(wrong["t"].view(np.uint64), right["t"].view(np.uint64))
                assert (kinds[right["object"][off]] == 1).all()
            else:  # only triangle indices move, none of them on a mesh hit
                assert np.array_equal(wrong["object"], right["object"]) and (kinds[right["object"][off]] != 2).all() and (wrong["triangle"][off] != 0).all()
                on_planes += int((kinds[right["object"][off]] == 0).sum())
        print("rays host: %s changes %d records of %s" % (variant, differ, rs.label))
        assert differ > 0, variant
        assert variant != "triangle_kept_off_the_mesh" or on_planes > 0  # a plane in front of a mesh hit


# ---------------------------------------------------------------- 4: raymond_cli's arguments, which need no device
@pytest.fixture(scope="module")
def cli(product_lib):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raymond_amd", "host")], check=True)
    return CLI


def test_cli_pick_argument_handling(cli):
    def refused(word, *args):
        r = subprocess.run([cli, "pick"] + list(args), capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr and not r.stdout, (args, r.stderr)

    refused("SCENE --pixel X,Y")
    refused("--pixel X,Y is needed", "spheres")
    refused("SCENE --pixel X,Y", "spheres", "--pixel")  # an option without its value
    refused("2 comma-separated values", "spheres", "--pixel", "3")
    refused("2 comma-separated values", "spheres", "--pixel", "3,4,5")
    refused("not an unsigned integer", "spheres", "--pixel", "3,x")
    refused("not an unsigned integer", "spheres", "--pixel", "-3,4")
    refused("not a number", "spheres", "--pixel", "3,4 ")
    refused("above 2^32 - 1", "spheres", "--pixel", "4294967296,0")
    refused("pixel outside the frame", "spheres", "--pixel", "1920,0")
    refused("pixel outside the frame", "spheres", "--pixel", "0,1080")
    refused("pixel outside the frame", "spheres", "--pixel", "8,0", "--size", "8,6")
    refused("1..65535 per axis", "spheres", "--pixel", "0,0", "--size", "0,6")
    refused("1..65535 per axis", "spheres", "--pixel", "0,0", "--size", "8,65536")
    refused("not a number", "spheres", "--pixel", "0,0", "--fov", "wide")
    refused("3 comma-separated values", "spheres", "--pixel", "0,0", "--position", "0,0")
    refused("unknown option --bogus", "spheres", "--pixel", "0,0", "--bogus", "1")
    refused("unknown scene nosuch", "nosuch", "--pixel", "0,0")  # after the options, before a device
    text = open(os.path.join(ROOT, "raymond_amd", "host", "cli.cpp")).read()
    assert '"object triangle t nx ny nz"' in text and "%.17g" in text.split("raymond_cli pick SCENE", 1)[1].split("raymond_cli display-weights", 1)[0]  # the printed format is in the help text


def test_cli_intersect_file_size_refusals(cli, tmp_path):
    out = tmp_path / "out.hits"

    def run(*args):
        return subprocess.run([cli, "intersect"] + [str(a) for a in args], capture_output=True, text=True)

    for n_bytes in (8, 47, 49, 48 * 3 + 40):
        (tmp_path / "bad.f64").write_bytes(b"\0" * n_bytes)
        r = run("spheres", "--rays", tmp_path / "bad.f64", "--out", out)
        assert r.returncode == 1 and "no whole number of 48-byte rays" in r.stderr and str(n_bytes) in r.stderr and not out.exists(), r.stderr
    r = run("spheres", "--rays", tmp_path / "absent.f64", "--out", out)
    assert r.returncode == 1 and "cannot read" in r.stderr and not out.exists()
    for args in (("spheres",), ("spheres", "--rays", tmp_path / "bad.f64"), ("spheres", "--out", out)):
        r = run(*args)
        assert r.returncode == 1 and "--rays and --out are both needed" in r.stderr, (args, r.stderr)
    r = run("spheres", "--rays")
    assert r.returncode == 1 and "SCENE --rays IN.f64 --out OUT.hits" in r.stderr
    r = run("spheres", "--rays", tmp_path / "bad.f64", "--out", out, "--bogus", "1")
    assert r.returncode == 1 and "unknown option --bogus" in r.stderr
    (tmp_path / "none.f64").write_bytes(b"")
    r = run("spheres", "--rays", tmp_path / "none.f64", "--out", out)  # no rays: an empty file of records, and no device is asked for
    assert r.returncode == 0 and r.stdout == "0 rays, 0 hits\n" and out.read_bytes() == b""
