"""The tile classes of the spheres kernel's work items (raymond_amd/csrc/primary_candidates.hpp: TILE CLASSES), on the GPU.

An EMITTER item stores the wall's colour for every sample without a random number or a ray; a BLACK item draws block 0 first and makes rays for the survivors only
(render_kernel.hpp: render_wave_sorted).  Neither changes a bit of the frame:
  * frames rendered with RMD_TUNE_AXIS_PAIRS at 0 (classes on) and at 3 (every item general) are identical byte for byte — a 64x64 crop of C1's
    frame and whole frames of 96x80 and 93x77 (ragged rect and wave tiles), at 3 and 33 samples per pixel (an item shorter than one round; pairs
    that are no multiple of a round), bounce limits 1, 2 and 5, in the automatic launch (the direct mode at these sizes; at 130 samples per pixel the buffered one), with items of ONE sample
    (RMD_TUNE_SPLIT_MIN_SAMPLES = 1: an item shorter than a round) and with forced splits of 2 and 4;
  * likewise with sample_begin != 0, with RMD_RENDER_TRACE_BLACK_PATHS (no class at all), through rmd_render_tiles_moments (sum and squares), under
    the thin lens (general), and for cameras that make the whole frame EMITTER (the back wall emits) and the whole frame BLACK — where the host
    probe says so;
  * in the DIAG build at 64x64 (RMD_DEBUG bits 8 | 512, whole and tail items both: bit 1024) every sample a class ends without a ray has its full
    path — jitter, ray, the full visit, the classification's rule — run beside it: no sample disagrees and no ray hits another object than the
    predicted wall, while the class counts are what the frames were built to have; and the frames are identical there too.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from raymond_amd import abi, probe, render, scenes
from raymond_amd.scene import CameraSettings, Material, Object, Plane, Settings, Transform, generate_tiles
from test_primary_candidates import wave_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "raymond_amd", "csrc", "diag", "libraymond_hip.so")
ON, OFF = 0, 3  # RMD_TUNE_AXIS_PAIRS: the library's choice; the candidate sets without the tile classes


def emitting_back_wall():
    """reflective_spheres with the back wall (z = 5) an emitter: an emitter that is not the ceiling"""
    sc = scenes.reflective_spheres()
    i = next(i for i, o in enumerate(sc.objects) if isinstance(o.geometry, Plane) and tuple(o.geometry.normal) == (0.0, 0.0, -1.0))
    sc.objects[i] = Object(sc.objects[i].geometry, Material.Emission((0.25, 1.0, 3.5)))
    return sc


# a narrow view from above the spheres: every wave tile of the frame sees the back wall and nothing else
ONE_WALL_CAMERA = dict(fov=12.0, pos=(0.0, 1.2, 0.0))


def one_wall_camera(W, H):
    return CameraSettings(W, H, ONE_WALL_CAMERA["fov"], Transform(ONE_WALL_CAMERA["pos"]))


def frames(ctx, scene, st, switch, tiles=None, moments=False, split=0, sample_begin=0, sample_count=None):
    """(sum, squares or None) of one render with RMD_TUNE_AXIS_PAIRS = switch.  split: 0 = the automatic launch, 2 / 4 = RMD_TUNE_SAMPLE_SPLIT (which
    keeps four samples an item: at 3 samples per pixel it is the direct mode), -1 = the automatic launch with RMD_TUNE_SPLIT_MIN_SAMPLES = 1: as many
    items per wave tile as it has samples (up to 64), each shorter than one generation round."""
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    ctx.set_tunable(abi.RMD_TUNE_AXIS_PAIRS, switch)
    ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, max(split, 0))
    ctx.set_tunable(abi.RMD_TUNE_SPLIT_MIN_SAMPLES, 1 if split < 0 else 0)
    try:
        ds = render.DeviceScene(ctx, scene)
        fb = render.Framebuffer(ctx, W, H)
        fb_sq = render.Framebuffer(ctx, W, H) if moments else None
        try:
            render.render_tiles(ctx, ds, cam, st, tiles if tiles is not None else generate_tiles(W, H, st.tile_size), fb, sample_begin=sample_begin,
                                sample_count=sample_count, framebuffer_sq=fb_sq)
            info = ctx.last_launch_info()
            n = st.sample_count if sample_count is None else sample_count
            # the role-sorted kernel (buffered) wherever the launch rules give it: a forced split of at least four samples an item, items of one sample,
            # the automatic launch from 128 samples per pixel; else the direct mode, where no item has a class and the comparison is of the switch alone
            buffered = (split < 0 and n >= 2) or (split > 0 and n >= 8) or (split == 0 and n >= 128)
            assert info.has_grid == 0 and info.buffered == (1 if buffered else 0), (split, n, info.buffered)
            return fb.download(), (fb_sq.download() if moments else None)
        finally:
            fb.close()
            if fb_sq is not None:
                fb_sq.close()
            ds.close()
    finally:
        ctx.set_tunable(abi.RMD_TUNE_AXIS_PAIRS, 0)
        ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0)
        ctx.set_tunable(abi.RMD_TUNE_SPLIT_MIN_SAMPLES, 0)


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def base_frame(name):
    """-> (camera, tile rects): C1's frame cropped to 64x64 — ceiling, back wall and the top of a sphere —, or a whole small frame"""
    if name == "c1_crop":
        cam = scenes.camera(256, 256)
        return cam, [(x, y, 32, 32) for y in (0, 32) for x in (96, 128)]
    W, H = {"96x80": (96, 80), "93x77": (93, 77)}[name]
    return scenes.camera(W, H), generate_tiles(W, H, (32, 32))


@pytest.mark.parametrize("frame", ["c1_crop", "93x77"])
def test_frames_are_identical_in_the_automatic_launch_of_the_role_sorted_kernel(gpu_ctx, frame):
    """130 samples per pixel: the automatic launch is the buffered one (frames() asserts it) — at 3 and 33 it is the direct mode"""
    cam, tiles = base_frame(frame)
    st = Settings(cam, sample_count=130, tile_size=(32, 32), bounce_limit=5, seed=scenes.SEED)
    sc = scenes.reflective_spheres()
    a, _ = frames(gpu_ctx, sc, st, ON, tiles=tiles)
    b, _ = frames(gpu_ctx, sc, st, OFF, tiles=tiles)
    assert np.isfinite(a).all() and a.max() > 0.0 and same_bytes(a, b)


@pytest.mark.parametrize("split", [0, -1, 2, 4])
@pytest.mark.parametrize("bounces", [1, 2, 5])
@pytest.mark.parametrize("spp", [3, 33])
@pytest.mark.parametrize("frame", ["c1_crop", "96x80", "93x77"])
def test_frames_are_identical_with_the_tile_classes_on_and_off(gpu_ctx, frame, spp, bounces, split):
    cam, tiles = base_frame(frame)
    st = Settings(cam, sample_count=spp, tile_size=(32, 32), bounce_limit=bounces, seed=scenes.SEED)
    sc = scenes.reflective_spheres()
    if split == 2 and spp == 33 and bounces == 5:  # the frame was built to hold both classes (the host probe: the kernel's own functions)
        W, H = cam.backbuffer_width, cam.backbuffer_height
        wt = np.array([(x, y, min(8, min(tx + tw, W) - x), min(8, min(ty + th, H) - y)) for tx, ty, tw, th in tiles for y in range(ty, min(ty + th, H), 8) for x in range(tx, min(tx + tw, W), 8)], dtype=np.uint32)
        on, cls, _ = probe.tile_classes(cam, st, sc, wt)
        assert on and (cls == probe.TILE_EMITTER).any() and (cls == probe.TILE_BLACK).any() and (cls == probe.TILE_GENERAL).any()
    a, _ = frames(gpu_ctx, sc, st, ON, tiles=tiles, split=split)
    b, _ = frames(gpu_ctx, sc, st, OFF, tiles=tiles, split=split)
    assert np.isfinite(a).all() and a.max() > 0.0
    assert same_bytes(a, b)


@pytest.mark.parametrize("split", [-1, 2, 4])
@pytest.mark.parametrize("variant", ["sample_begin", "trace_black_paths", "moments", "all_emitter", "all_black", "lens"])
def test_variants_are_identical_with_the_tile_classes_on_and_off(gpu_ctx, variant, split):
    W, H, spp = 64, 64, 33
    cam, sc, kw, flags = scenes.camera(W, H), scenes.reflective_spheres(), {}, {}
    expect = None
    if variant == "sample_begin":
        kw = dict(sample_begin=7, sample_count=26)
    elif variant == "trace_black_paths":
        flags, expect = dict(trace_black_paths=True), "off"
    elif variant == "all_emitter":
        cam, sc, expect = one_wall_camera(W, H), emitting_back_wall(), probe.TILE_EMITTER
    elif variant == "all_black":
        cam, expect = one_wall_camera(W, H), probe.TILE_BLACK
    elif variant == "lens":
        cam, flags, expect = scenes.camera(W, H, aperture_radius=0.05), dict(use_dof=True), "off"
    st = Settings(cam, sample_count=spp, tile_size=(32, 32), bounce_limit=4, seed=scenes.SEED + 1, **flags)
    on, cls, _ = probe.tile_classes(cam, st, sc, wave_tiles(W, H))
    if expect == "off":
        assert not on and (cls == probe.TILE_GENERAL).all()
    elif expect is not None:
        assert on and (cls == expect).all()
    a, a_sq = frames(gpu_ctx, sc, st, ON, moments=variant == "moments", split=split, **kw)
    b, b_sq = frames(gpu_ctx, sc, st, OFF, moments=variant == "moments", split=split, **kw)
    assert np.isfinite(a).all() and same_bytes(a, b)
    if variant == "moments":
        assert same_bytes(a_sq, b_sq) and a_sq.max() > 0.0
    if variant == "all_emitter":  # every pixel is spp times the colour, added one sample at a time
        want = np.zeros(3)
        for _ in range(spp):
            want = want + np.array([0.25, 1.0, 3.5])
        assert (a == want[None, None, :]).all()


DIAG_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np
import test_gpu_tile_classes as T
from raymond_amd import abi, lib, render, scenes
from raymond_amd.scene import Settings, generate_tiles

assert lib.LIB_PATH.endswith("diag/libraymond_hip.so"), lib.LIB_PATH
# 8: event counters, 512: every sample a class ends has its full path run beside it, 1024: the work list's tail is 4 wave tiles (whole items too)
os.environ["RMD_DEBUG"] = "1544"

def run(name, scene, cam, spp, split, tiles=None):
    st = Settings(cam, sample_count=spp, tile_size=(32, 32), bounce_limit=5, seed=scenes.SEED)
    out = []
    for switch in (T.ON, T.OFF):
        with render.Context(0) as ctx:
            ctx.set_tunable(abi.RMD_TUNE_LAUNCH_FORM, 2)  # persistent, however few the items
            sys.stderr.write("== %%s %%s\n" %% (name, "on" if switch == T.ON else "off")), sys.stderr.flush()
            out.append(T.frames(ctx, scene, st, switch, tiles=tiles, split=split)[0])
            info = ctx.last_launch_info()
            assert info.buffered == 1 and info.persistent == 1, name
    assert T.same_bytes(out[0], out[1]), name

for spp, split in ((130, 0), (33, 2)):
    tag = "whole" if split == 0 else "split"
    run("mixed " + tag, scenes.reflective_spheres(), *T.base_frame("c1_crop")[:1], spp, split, tiles=T.base_frame("c1_crop")[1])  # ceiling, back wall, a sphere
    run("emitter " + tag, T.emitting_back_wall(), T.one_wall_camera(64, 64), spp, split)
    run("black " + tag, scenes.reflective_spheres(), T.one_wall_camera(64, 64), spp, split)
print("tile classes ok")
"""

CLASS_LINE = (r"tile classes: general items=(\d+) emitter items=(\d+) black items=(\d+) \| black rounds=(\d+) cut short=(\d+) samples ended in pass A=(\d+) "
              r"survivors=(\d+) \| samples checked against their full path=(\d+) .*\(must be 0\)=(\d+) .*\(must be 0\)=(\d+)")
CLASS_KEYS = ("general", "emitter", "black", "rounds", "cut", "ended", "survivors", "checked", "bad_samples", "bad_rays")


def test_class_ended_samples_agree_with_their_full_path_in_the_diag_build(product_lib):
    assert os.path.exists(DIAG_LIB), "build the DIAG library: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, RAYMOND_HIP_LIB=DIAG_LIB)
    env.pop("RMD_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", DIAG_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "tile classes ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    seen, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("== "):
            name = line[3:]
        m = re.search(CLASS_LINE, line)
        if m and name:
            d = seen.setdefault(name, dict.fromkeys(CLASS_KEYS, 0))
            for k, v in zip(CLASS_KEYS, m.groups()):
                d[k] += int(v)
    print(seen)
    assert len(seen) == 12, r.stderr[-3000:]
    for name, d in seen.items():
        assert d["bad_samples"] == 0 and d["bad_rays"] == 0, (name, d)
        if name.endswith(" off"):
            assert d["emitter"] == 0 and d["black"] == 0 and d["general"] > 0 and d["checked"] == 0, (name, d)
            continue
        spp = 130 if "whole" in name else 33
        if name.startswith("mixed"):
            assert d["general"] > 0 and d["emitter"] > 0 and d["black"] > 0, (name, d)
        if name.startswith("emitter"):
            assert d["general"] == 0 and d["black"] == 0 and d["emitter"] > 0 and d["checked"] == 64 * 64 * spp, (name, d)
        if name.startswith("black"):
            assert d["general"] == 0 and d["emitter"] == 0 and d["black"] > 0, (name, d)
            assert d["ended"] + d["survivors"] == 64 * 64 * spp and d["checked"] == d["ended"], (name, d)
            assert 0.45 < d["ended"] / (64 * 64 * spp) < 0.55, (name, d)  # lobe_bits is a 22-bit uniform
        if d["black"] > 0:
            assert d["rounds"] > 0 and d["ended"] > 0 and d["survivors"] > 0 and d["checked"] >= d["ended"], (name, d)
    # whole items and tail items both occurred (bit 1024: all but 4 of the 64 wave tiles are whole items in the automatic launch)
    assert 64 < seen["emitter whole on"]["emitter"] < 128 and seen["emitter split on"]["emitter"] == 64 * 2, seen
