"""The candidate sets of the spheres kernel's generation trips (raymond_amd/csrc/primary_candidates.hpp), on the GPU.

  * frames rendered with RMD_TUNE_AXIS_PAIRS at 0 (the candidate sets on) and at 2 (off) are identical byte for byte: C1 and the whole C2 frame, in
    the default mode, with RMD_RENDER_TRACE_BLACK_PATHS, and through rmd_render_tiles_moments for both the sum and the squares;
  * a launch under the thin lens and a scene outside the regular parameter class — where the sets are off anyway — are identical too;
  * in the DIAG build (RMD_DEBUG bits 8 | 512) every generation trip also runs the full visit: no cleared sphere registers a hit and no closest
    (distance, object) differs, over the whole C2 frame and over frames whose camera sits close to a sphere — while spheres and pairs ARE left out.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from raymond_amd import abi, render, scenes
from raymond_amd.scene import CameraSettings, Material, Object, Settings, Sphere, Transform, generate_tiles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "raymond_amd", "csrc", "diag", "libraymond_hip.so")


def frames(ctx, scene, st, switch, moments=False, split=0):
    """(sum, squares or None) of one render with RMD_TUNE_AXIS_PAIRS = switch (read when the scene is created)."""
    cam = st.camera_settings
    W, H = cam.backbuffer_width, cam.backbuffer_height
    ctx.set_tunable(abi.RMD_TUNE_AXIS_PAIRS, switch)
    ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, split)
    try:
        ds = render.DeviceScene(ctx, scene)
        fb = render.Framebuffer(ctx, W, H)
        fb_sq = render.Framebuffer(ctx, W, H) if moments else None
        try:
            render.render_tiles(ctx, ds, cam, st, generate_tiles(W, H, st.tile_size), fb, framebuffer_sq=fb_sq)
            info = ctx.last_launch_info()
            assert info.buffered == 1 and info.has_grid == 0  # the role-sorted spheres kernel: the one with generation trips
            return fb.download(), (fb_sq.download() if moments else None)
        finally:
            fb.close()
            if fb_sq is not None:
                fb_sq.close()
            ds.close()
    finally:
        ctx.set_tunable(abi.RMD_TUNE_AXIS_PAIRS, 0)
        ctx.set_tunable(abi.RMD_TUNE_SAMPLE_SPLIT, 0)


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["C1", "C2"])
@pytest.mark.parametrize("mode", ["default", "trace_black_paths", "moments"])
def test_frames_are_identical_with_the_candidate_sets_on_and_off(gpu_ctx, name, mode):
    st = scenes.config_settings(name)
    st.trace_black_paths = mode == "trace_black_paths"
    split = 2 if name == "C1" else 0  # (C1's 16 samples per pixel take the direct mode by default: the split launch is asked for)
    sc = scenes.reflective_spheres()
    on, on_sq = frames(gpu_ctx, sc, st, 0, moments=mode == "moments", split=split)
    off, off_sq = frames(gpu_ctx, sc, st, 2, moments=mode == "moments", split=split)
    assert np.isfinite(on).all() and on.max() > 0.0
    assert same_bytes(on, off)
    if mode == "moments":
        assert same_bytes(on_sq, off_sq) and on_sq.max() > 0.0


def test_a_thin_lens_launch_and_an_irregular_scene_are_identical(gpu_ctx):
    W, H = 256, 256
    cam = scenes.camera(W, H, aperture_radius=0.05)
    st = Settings(cam, sample_count=130, bounce_limit=4, seed=scenes.SEED, use_dof=True)
    sc = scenes.reflective_spheres()
    a, _ = frames(gpu_ctx, sc, st, 0)
    b, _ = frames(gpu_ctx, sc, st, 2)
    assert same_bytes(a, b) and a.max() > 0.0
    irregular = scenes.reflective_spheres()
    irregular.objects.append(Object(Sphere((0.3, 0.8, 2.5), 0.3), Material.Metal((1.0, 1.0, 1.0), 0.0)))  # roughness 0: outside the regular class
    st2 = Settings(scenes.camera(W, H), sample_count=130, bounce_limit=4, seed=scenes.SEED)
    a, _ = frames(gpu_ctx, irregular, st2, 0)
    b, _ = frames(gpu_ctx, irregular, st2, 2)
    assert same_bytes(a, b)


DIAG_CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r)
from raymond_amd import lib, render, scenes
from raymond_amd.scene import CameraSettings, Settings, Transform, generate_tiles

assert lib.LIB_PATH.endswith("diag/libraymond_hip.so"), lib.LIB_PATH
os.environ["RMD_DEBUG"] = "520"  # 8: event counters, 512: every generation trip ALSO runs the full visit and is compared with it

def run(name, cam, spp, bounces=5):
    with render.Context(0) as ctx:
        st = Settings(cam, sample_count=spp, bounce_limit=bounces, seed=scenes.SEED)
        W, H = cam.backbuffer_width, cam.backbuffer_height
        ds, fb = render.DeviceScene(ctx, scenes.reflective_spheres()), render.Framebuffer(ctx, W, H)
        sys.stderr.write("== %%s\n" %% name), sys.stderr.flush()
        render.render_tiles(ctx, ds, cam, st, generate_tiles(W, H, st.tile_size), fb)
        info = ctx.last_launch_info()
        assert info.buffered == 1 and info.has_grid == 0, name
        fb.close(), ds.close()

c2 = scenes.config_settings("C2")
run("C2", c2.camera_settings, c2.sample_count, c2.bounce_limit)
# cameras close to the spheres of the scene ((-1, -0.5, 3.5) r 0.5 and (0.74, -0.25, 3.5) r 0.75): just outside, grazing, and inside one
run("outside sphere 0", CameraSettings(320, 200, 70.0, Transform((-1.0, -0.5, 2.99))), 130)
run("beside sphere 1", CameraSettings(320, 200, 100.0, Transform((-0.02, -0.25, 3.3))), 130)
run("inside sphere 1", CameraSettings(200, 320, 55.0, Transform((0.74, -0.25, 3.2))), 130)
print("candidates ok")
"""


def test_the_full_visit_agrees_with_the_candidate_visit_in_the_diag_build(product_lib):
    assert os.path.exists(DIAG_LIB), "build the DIAG library: python -c 'import __graft_entry__ as g; g.build()'"
    env = dict(os.environ, RAYMOND_HIP_LIB=DIAG_LIB)
    env.pop("RMD_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", DIAG_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0 and "candidates ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    seen, name = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("== "):
            name = line[3:]
        m = re.search(r"primary candidates: lanes checked=(\d+) sphere turns left out=(\d+) trips with two axis pairs left out=(\d+) .*\(must be 0\)=(\d+) .*\(must be 0\)=(\d+)", line)
        if m and name:
            d = seen.setdefault(name, dict(lanes=0, turns=0, pair_trips=0, wrong=0, differs=0))
            for k, v in zip(("lanes", "turns", "pair_trips", "wrong", "differs"), m.groups()):
                d[k] += int(v)
    print(seen)
    assert len(seen) == 4, r.stderr[-3000:]
    for name, d in seen.items():
        assert d["wrong"] == 0 and d["differs"] == 0, (name, d)
        assert d["lanes"] > 0, (name, d)
    assert seen["C2"]["lanes"] == 1920 * 1080 * 500
    for name in ("C2", "outside sphere 0", "beside sphere 1"):
        assert seen[name]["turns"] > 0 and seen[name]["pair_trips"] > 0, (name, seen[name])  # it ran, and it left objects out
